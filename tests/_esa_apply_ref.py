"""The ESA apply, y = x * sigmoid(conv4(bilinear(c3) + conv_f(c1))) (esr_esa_apply_f32), restated for the tests:

  ref64       the operation in fp64 on the values the kernel reads, with the per-element error bound of a correct kernel
  emulate32   the documented arithmetic of esa_apply_mfma_kernel in torch fp32 -- the kernel's stand-in on a host without a GPU --
              and, by name, the ways that arithmetic can be subtly wrong (MUTANTS)
  compare     the assertions every value test of the op makes: (a) a per-element bound, (b) the share of stored values that are not the
              correctly rounded reference, and -- where the emulation is handed in -- (c) the share that differs from the emulation

Everything is NHWC: x [N,H,W,c] and c1 [N,H,W,f] in the storage type (fp32, bf16, fp16), c3 [N,h_lo,w_lo,f] fp32, wf [f,f] and
w4 [c,f] as (out, in), bf [f], b4 [c].  tests/test_esa_apply_ref.py proves on the CPU that emulate32 passes compare() and that every
mutant fails it; tests/test_gpu_esa_apply.py holds the kernels to it.

Bound (a), 16-bit storage.  sigma' <= 1/4, so |y - ref| <= |x| * dm / 4 + (fp32 sigmoid and product) + (the store's rounding), where dm
bounds the error of the gate's argument m.  With u = 2^-24 and P = 16 (bf16) / 22 (fp16) significant bits of a value kept as a high
and a low 16-bit part -- p = 8 / 11 significant bits each: |v - hi| <= 2^-p |v|, and the low part rounds that remainder again,
|v - (hi + lo)| <= 2^-2p |v| = 2^-P |v| -- plus, for fp16 only, half the subnormal step, 2^-25 (a low part below 2^-14 is a
subnormal; bf16 has fp32's exponent range).  The kernel drops the product of the two low parts, |w_lo s_lo| <= 2^-P |w| |s|:

  ferr(v) = 2^-P |v| + sub
  A_k  = sum_i |wf_ki| |c1_i| + |up_k| + |bf_k|                the terms of s_k
  ds_k = sum_i ferr(wf_ki) |c1_i|                              Wf as hi + lo against c1 as stored
       + (2 f + 8) u A_k                                       one fp32 rounding per product added (f high, f low) and per operation of the lerp
       + ct                                                    fp32 source coordinates, below
  B_c  = sum_k |w4_ck| |s_k| + |b4_c|
  dm_c = sum_k |w4_ck| (ds_k + ferr(s_k))                      s as computed, then as hi + lo
       + sum_k ferr(w4_ck) |s_k|                               W4 as hi + lo
       + 2^-P sum_k |w4_ck| |s_k|                              W4_lo s_lo, not computed
       + (3 f + 2) u B_c                                       one fp32 rounding per product added, and the bias
  arith = |x| dm / 4 + 8 u |ref|                               (v_exp, v_rcp, 1 + e, the product: a few fp32 roundings)
  bound = max(1.01 * eps * |ref|, smallest step / 2) + arith   eps = 2^-8 / 2^-11: half a step, the factors of test_gpu_h16._ulp_ok

ct: the kernels compute fy = fmaf(oy + 0.5, float(h_lo) / float(H), -0.5) in fp32.  The scale is rounded once (relative u), the fmaf
once (u * fy), and fy < h_lo, so |fy - exact| <= 2 u h_lo = 2^-23 h_lo; ly = fy - floor(fy) is exact.  Bilinear interpolation is
continuous and piecewise linear with slope <= the largest difference of vertical neighbours Dy, so up moves by at most 2^-23 h_lo Dy,
likewise 2^-23 w_lo Dx: ct = 2^-23 (h_lo Dy + w_lo Dx), one scalar per case.

fp32 storage keeps the suite's 2e-5 * max(1, max|ref|) and adds the same coordinate term, |x| / 4 * ct * sum_k |w4_ck|.

Check (b), 16-bit storage.  A stored value differs from RNE(ref) only if ref lies within `arith` of a rounding boundary; boundaries are
one step apart, so for ref spread evenly over a step the chance is min(1, 2 arith / step) and the expected number of such values is
E = sum_i min(1, 2 arith_i / step_i).  compare() allows E + 4 sqrt(E) + 4: the count is a sum of independent 0 / 1 draws of mean <= E,
so its variance is <= E; four standard deviations, and + 4 because for E below ~1 the count is Poisson-like, not normal.  Every such value
may differ by ONE step.  (a) alone would let an error of half a step through wherever the rounding leaves room; (b) counts how often the
rounding itself went the other way.  E is a worst-case figure (every error at its bound, all of one sign): the emulation and the
kernels stay two orders of magnitude below it, see DESIGN.md section 2f for what each mutant does to both figures.

Check (c), 16-bit storage: the kernel against emulate32.  Both evaluate the SAME expression on the same fp32 numbers -- the same source
coordinates, lerp, splits and dropped product -- and may differ only where fp32 sums are rounded (the order in which a matrix instruction
adds its products is not documented) and in the sigmoid's last bits.  So of `arith` only the fp32 terms remain, once per side:

  ds32_k  = (2 f + 8) u A_k
  arith32 = |x| / 4 (sum_k |w4_ck| ds32_k + (3 f + 2) u B_c) + 8 u |ref|     two evaluations lie within 2 arith32 of each other

and one thing is added: if the two sides' s_k fall on different sides of a 16-bit boundary (chance q_k = min(1, 2 ds32_k / step(s_k))),
their high parts differ by a step, hi + lo still represents s_k to 2^-P, but W4_lo s_hi and the dropped W4_lo s_lo move by up to
2^-P |w4_ck| |s_k| each and the representation error by as much again: a displacement of 3 * 2^-P |w4_ck| |s_k| with probability q_k,

  extra = |x| / 4 * 3 * 2^-P sum_k q_k |w4_ck| |s_k|

A stored value differs when a rounding boundary lies between the two pre-rounding values: expected count E32 = sum_i min(1, 2 (arith32_i
+ extra_i) / step_i), allowed E32 + 4 sqrt(E32) + 4 as in (b), each by one step.  E32 is 0.4 - 6 % of the values in bf16 and
3 - 24 % in fp16 on the cases of the GPU matrix, against the 10 - 22 % that a dropped low-part image flips: in bf16 this is the check
that sees an error far below half a step.  tests/test_esa_apply_ref.py shows that it lets a different summation through (fp64 sums rounded once)."""
import math

import torch

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
EPS = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}              # half a step relative to the binade's lower end
PBITS = {"bf16": 16, "f16": 22}                           # significant bits of hi + lo
MBITS = {"bf16": 7, "f16": 10}                            # stored mantissa bits
EMIN = {"bf16": -126, "f16": -14}                         # exponent of the smallest normal
U = 2.0 ** -24

# geometries (n, h, w, (h_lo, w_lo)) and widths (c, f) of the GPU matrix; tests/test_esa_apply_ref.py uses them too
GEOMS = [(2, 15, 15, (1, 1)), (3, 5, 8, (1, 1)), (2, 19, 8, (3, 1)), (2, 12, 9, (2, 2)), (2, 23, 37, (5, 8)), (1, 33, 17, (4, 1)),
         (1, 20, 36, (1, 4)), (1, 1, 90, (1, 7)), (1, 16, 24, (16, 24)), (1, 32, 32, (16, 16)), (1, 10, 12, (25, 31))]
WIDTHS = [(20, 8), (32, 16), (33, 16), (42, 10), (46, 16), (50, 12), (64, 16)]
BIG = (5, 480, 450, (78, 73))


def combos():
    """every width on the first, fifth and tenth geometry; every geometry on (50, 12) and (32, 16) -- not the full product"""
    out = []
    for gi, g in enumerate(GEOMS):
        for wd in WIDTHS:
            if gi in (0, 4, 9) or wd in ((50, 12), (32, 16)):
                out.append((g, wd))
    return out


def case_id(g, wd):
    n, h, w, lo = g
    return f"{n}x{h}x{w}-lo{lo[0]}x{lo[1]}-c{wd[0]}f{wd[1]}"


def make_inputs(geom, width, storage, seed=0):
    """x ~ 3 randn and c1 ~ randn rounded to the storage type, c3 ~ randn fp32, wf, w4 ~ 0.3 randn, non-zero biases (CPU tensors)"""
    n, h, w, (hl, wl) = geom
    c, f = width
    g = torch.Generator().manual_seed(seed + 1000 * c + 10 * f + h + 7 * w)
    dt = DTYPES[storage]
    return dict(x=(torch.randn(n, h, w, c, generator=g) * 3).to(dt), c1=torch.randn(n, h, w, f, generator=g).to(dt),
                c3=torch.randn(n, hl, wl, f, generator=g), wf=torch.randn(f, f, generator=g) * 0.3, bf=torch.randn(f, generator=g) * 0.5,
                w4=torch.randn(c, f, generator=g) * 0.3, b4=torch.randn(c, generator=g) * 0.5)


# ---- pixel coordinates -------------------------------------------------------------------------------------------------------------------
def exact_coords(N, H, W, device="cpu"):
    pix = torch.arange(N * H * W, device=device)
    return pix // (H * W), (pix // W) % H, pix % W


def carry_coords(N, H, W, wraps=2):
    """(n, oy, ox) of every pixel as both apply kernels derive them: one division chain for the first pixel of a group of 16 consecutive
    pixels, + the lane, carried over at most `wraps` image rows.  Equal to exact_coords for W >= 8 with the kernels' two wraps."""
    pix = torch.arange(N * H * W)
    pix0 = pix // 16 * 16
    row0 = pix0 // W
    n = row0 // H
    ox = pix0 - row0 * W + (pix - pix0)
    oy = row0 - n * H
    for _ in range(wraps):
        m = ox >= W
        ox = ox - W * m
        oy = oy + m
        m2 = m & (oy == H)
        oy = torch.where(m2, torch.zeros_like(oy), oy)
        n = n + m2
    return n, oy, ox


# ---- bilinear source index ---------------------------------------------------------------------------------------------------------------
def _src(dst, inn, out, *, fp32, mutant=None):
    """ATen's area_pixel_compute_source_index, align_corners=False: scale (dst + 0.5) - 0.5 with scale = in / out, clamped at 0; the upper
    neighbour clamped at the edge.  dst: integer tensor (any value: a mutant's column may lie past the row).  fp32: as the kernels compute
    it (scale rounded to fp32, one fmaf).  Returns (i0, i1, lambda) with lambda in the dtype of the arithmetic."""
    d = dst.double()
    if fp32:
        scale = float(torch.tensor(float(inn), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32))
    else:
        scale = inn / out
    if mutant == "align_corners":
        scale = (inn - 1) / (out - 1) if out > 1 else 0.0
        if fp32:
            scale = float(torch.tensor(scale, dtype=torch.float32))
        fy = d * scale
    elif mutant == "no_half_pixel":
        fy = d * scale
    else:
        fy = (d + 0.5) * scale - 0.5              # fp64: the product of two 24-bit numbers is exact, so rounding this once IS the fmaf
    if fp32:
        fy = fy.float()
    if mutant != "no_clamp0":
        fy = fy.clamp(min=0)
    i0 = fy.to(torch.int64)                       # (int) truncates, as the kernels' cast
    i1 = i0 + 1 if mutant == "no_clamp_edge" else i0 + (i0 < inn - 1).to(torch.int64)
    return i0, i1, fy - i0.to(fy.dtype)


def _taps(c3, n, oy, ox, H, W, *, fp32, mutant=None):
    """the four neighbours [P, f] of every pixel and (ly, lx) [P, 1]; indices are flat, as the kernels', so a mutant's column or row past
    the edge reads the next row / image (zeros behind the tensor)"""
    N, hl, wl, f = c3.shape
    y0, y1, ly = _src(oy, hl, H, fp32=fp32, mutant=mutant)
    x0, x1, lx = _src(ox, wl, W, fp32=fp32, mutant=mutant)
    flat = torch.cat([c3.reshape(-1, f), torch.zeros(1, f, dtype=c3.dtype, device=c3.device)])
    last = flat.shape[0] - 1

    def at(yy, xx):
        return flat[((n * hl + yy) * wl + xx).clamp(0, last)]
    if mutant == "swap_lx_ly":
        ly, lx = lx, ly
    return at(y0, x0), at(y0, x1), at(y1, x0), at(y1, x1), ly[:, None], lx[:, None]


class Ref:
    """ref [N,H,W,c] fp64, arith = the arithmetic part of bound (a), step = the storage step at |ref| (16-bit storage), bound = (a),
    arith32 = what two fp32 evaluations of the kernel's expression may differ by, halved (check (c))"""
    def __init__(self, ref, arith, step, bound, storage, arith32=None):
        self.ref, self.arith, self.step, self.bound, self.storage, self.arith32 = ref, arith, step, bound, storage, arith32


def ref64(x, c1, c3, wf, bf, w4, b4, *, storage, device=None):
    """The operation in fp64 on the stored inputs, and bound (a) (module docstring).  device: where to compute (default: where x lives)."""
    dev = x.device if device is None else device
    N, H, W, c = x.shape
    f = wf.shape[0]
    hl, wl = c3.shape[1:3]
    X, C1, C3 = x.to(dev).double().reshape(-1, c), c1.to(dev).double().reshape(-1, c1.shape[-1])[:, :f], c3.to(dev).double()[..., :f]
    Wf, Bf, W4, B4 = (t.to(dev).double() for t in (wf.reshape(f, f), bf, w4.reshape(c, f), b4))
    n, oy, ox = exact_coords(N, H, W, dev)
    a, b, cc, d, ly, lx = _taps(C3, n, oy, ox, H, W, fp32=False)
    up = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * cc + lx * d)
    del a, b, cc, d
    s = up + C1 @ Wf.T + Bf
    m = s @ W4.T + B4
    ref = X * torch.sigmoid(m)
    dy = float((C3[:, 1:] - C3[:, :-1]).abs().max()) if hl > 1 else 0.0
    dx = float((C3[:, :, 1:] - C3[:, :, :-1]).abs().max()) if wl > 1 else 0.0
    ct = 2.0 ** -23 * (hl * dy + wl * dx)
    w4sum = W4.abs().sum(dim=1)
    if storage == "f32":
        arith = X.abs() / 4 * ct * w4sum
        bound = 2e-5 * max(1.0, float(ref.abs().max())) + arith
        return Ref(ref.reshape(N, H, W, c), arith.reshape(N, H, W, c), None, bound.reshape(N, H, W, c), storage)
    p, sub = 2.0 ** -PBITS[storage], (2.0 ** -25 if storage == "f16" else 0.0)

    def ferr(v):
        return v.abs() * p + sub
    A = C1.abs() @ Wf.abs().T + up.abs() + Bf.abs()
    ds = C1.abs() @ ferr(Wf).T + (2 * f + 8) * U * A + ct
    B = s.abs() @ W4.abs().T + B4.abs()
    dm = (ds + ferr(s)) @ W4.abs().T + s.abs() @ ferr(W4).T + p * (s.abs() @ W4.abs().T) + (3 * f + 2) * U * B
    arith = X.abs() * dm / 4 + 8 * U * ref.abs()
    e = torch.frexp(ref.abs())[1].double() - 1                                   # floor(log2 |ref|)
    step = torch.exp2(e.clamp(min=EMIN[storage]) - MBITS[storage])
    smallest = 2.0 ** (EMIN[storage] - MBITS[storage])
    bound = (1.01 * EPS[storage] * ref.abs()).clamp(min=smallest / 2) + arith
    # (c): the fp32 terms alone + the chance that s_k's high part falls on the other side of a boundary
    ds32 = (2 * f + 8) * U * A
    step_s = torch.exp2((torch.frexp(s.abs())[1].double() - 1).clamp(min=EMIN[storage]) - MBITS[storage])
    q = (2 * ds32 / step_s).clamp(max=1)
    arith32 = X.abs() / 4 * (ds32 @ W4.abs().T + (3 * f + 2) * U * B + 3 * p * ((q * s.abs()) @ W4.abs().T)) + 8 * U * ref.abs()
    return Ref(ref.reshape(N, H, W, c), arith.reshape(N, H, W, c), step.reshape(N, H, W, c), bound.reshape(N, H, W, c), storage,
               arith32.reshape(N, H, W, c))


# ---- the MFMA kernel's arithmetic in torch fp32 -------------------------------------------------------------------------------------------
MUTANTS = ("wf_rounded", "w4_rounded", "s_rounded", "align_corners", "no_half_pixel", "no_clamp0", "no_clamp_edge", "swap_lx_ly",
           "quarter_lx_zero", "tiles_swapped", "one_wrap")


def emulate32(x, c1, c3, wf, bf, w4, b4, *, storage, mutant=None, exact_sums=False):
    """esa_apply_mfma_kernel as documented, on the CPU in fp32: coordinates from the two-wrap carry and one fp32 fmaf, the lerp in the
    kernel's order, Wf = hi + lo against c1 as stored, s = hi + lo, W4_hi s_hi + W4_hi s_lo + W4_lo s_hi, fp32 sigmoid, one RNE store.
    (The order in which a matrix instruction adds its products is not documented; torch's fp32 matmul stands for it.)
    mutant: one of MUTANTS -- the same with one thing wrong.
    exact_sums: each chain of matrix instructions adds its products in fp64 and rounds the sum to fp32 once -- another summation a
    correct kernel might have; check (c) must let it through."""
    assert mutant is None or mutant in MUTANTS
    dt = DTYPES[storage]
    assert dt != torch.float32 and x.dtype == dt
    N, H, W, c = x.shape
    f = wf.shape[0]

    def split(v):
        hi = v.to(dt).float()
        return hi, (v - hi).to(dt).float()
    n, oy, ox = carry_coords(N, H, W, wraps=1 if mutant == "one_wrap" else 2)
    a, b, cc, d, ly, lx = _taps(c3.float()[..., :f], n, oy, ox, H, W, fp32=True, mutant=mutant)
    hy, hx = 1 - ly, 1 - lx
    lxb = lx.expand(-1, f).clone()
    if mutant == "quarter_lx_zero":
        lxb[:, 0:4] = 0                                           # lane quarter kq = 0: lx * tb and lx * td come back as 0 (hx is right)
    sacc = hy * (hx * a + lxb * b) + ly * (hx * cc + lxb * d) + bf.float()
    wf_hi, wf_lo = split(wf.reshape(f, f).float())
    if mutant == "wf_rounded":
        wf_lo = torch.zeros_like(wf_lo)
    c1f = c1.float().reshape(-1, c1.shape[-1])[:, :f]
    if exact_sums:
        s = (sacc.double() + c1f.double() @ wf_hi.double().T + c1f.double() @ wf_lo.double().T).float()
    else:
        s = sacc + (c1f @ wf_hi.T + c1f @ wf_lo.T)
    s_hi, s_lo = split(s)
    if mutant == "s_rounded":
        s_lo = torch.zeros_like(s_lo)
    w4_hi, w4_lo = split(w4.reshape(c, f).float())
    if mutant == "w4_rounded":
        w4_lo = torch.zeros_like(w4_lo)
    if exact_sums:
        m = (b4.double() + s_hi.double() @ w4_hi.double().T + s_lo.double() @ w4_hi.double().T + s_hi.double() @ w4_lo.double().T).float()
    else:
        m = b4.float() + (s_hi @ w4_hi.T + s_lo @ w4_hi.T + s_hi @ w4_lo.T)
    if mutant == "tiles_swapped":
        # tile t <-> t ^ 1 of the channel map 32 (t >> 1) + 8 kq + 4 (t & 1) + r: channel ch gets the gate of ch ^ 4 (zero weights behind c)
        c8 = (c + 7) // 8 * 8
        mp = torch.zeros(m.shape[0], c8)
        mp[:, :c] = m
        m = mp[:, torch.arange(c8) ^ 4][:, :c]
    y = x.float().reshape(-1, c) * torch.sigmoid(m)
    return y.to(dt).reshape(N, H, W, c)


# ---- the comparator -----------------------------------------------------------------------------------------------------------------------
def _ordered(t):
    """16-bit patterns as integers in value order (so that neighbours differ by 1)"""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b < 0, -(b & 0x7FFF), b)


def measure(got, r, emu=None):
    """got [N,H,W,c] (storage type, or fp32) against a Ref (and, 16-bit storage, against the emulation's result): dict of figures;
    nothing asserted"""
    ref = r.ref.to(got.device)
    err = (got.double() - ref).abs()
    share = err / r.bound.to(got.device)
    i = int(share.argmax())
    out = dict(worst=float(err.max()), share_a=float(share.reshape(-1)[i]), at=i, n=ref.numel())
    if r.storage != "f32":
        want = ref.float().to(got.dtype)
        dist = (_ordered(got) - _ordered(want)).abs()
        E = float((2 * r.arith / r.step).clamp(max=1).sum())
        out.update(mism=int((dist != 0).sum()), far=int((dist > 1).sum()), expect=E, cap=E + 4 * math.sqrt(E) + 4)
        if emu is not None:
            de = (_ordered(got) - _ordered(emu.to(got.device))).abs()
            E32 = float((2 * r.arith32.to(got.device) / r.step.to(got.device)).clamp(max=1).sum())
            out.update(emu_mism=int((de != 0).sum()), emu_far=int((de > 1).sum()), expect32=E32, cap32=E32 + 4 * math.sqrt(E32) + 4)
    return out


def describe(what, fig):
    s = f"{what}: max|got - ref| = {fig['worst']:.3e} ({fig['share_a']:.3f} of bound (a))"
    if "mism" in fig:
        s += (f"; {fig['mism']} of {fig['n']} values are not RNE(ref) ({fig['mism'] / fig['n']:.4%}; cap (b) {fig['cap']:.1f} = "
              f"{fig['cap'] / fig['n']:.4%}), {fig['far']} by more than one step")
    if "emu_mism" in fig:
        s += (f"; {fig['emu_mism']} differ from the emulation ({fig['emu_mism'] / fig['n']:.4%}; cap (c) {fig['cap32']:.1f} = "
              f"{fig['cap32'] / fig['n']:.4%}), {fig['emu_far']} by more than one step")
    return s


def failures(fig):
    """which of the assertions the figures miss: subset of {"a", "b", "c"}"""
    bad = set()
    if not fig["share_a"] <= 1.0:
        bad.add("a")
    if "mism" in fig and (fig["far"] > 0 or fig["mism"] > fig["cap"]):
        bad.add("b")
    if "emu_mism" in fig and (fig["emu_far"] > 0 or fig["emu_mism"] > fig["cap32"]):
        bad.add("c")
    return bad


def compare(got, r, what, emu=None):
    """print the figures, then assert (a), (b) and -- with the emulation's result -- (c); returns the figures"""
    fig = measure(got, r, emu)
    print(describe(what, fig))
    # (a) every element inside its derived bound (module docstring)
    assert fig["share_a"] <= 1.0, describe(what, fig) + f" -- element {fig['at']}"
    if "mism" in fig:
        # (b) values that are not the correctly rounded reference: one step at most, and no more of them than bound (a)'s arithmetic part
        # explains -- E = sum min(1, 2 arith / step) -- plus 4 sqrt(E) + 4 of counting noise (variance of a sum of 0 / 1 draws <= its mean;
        # + 4 for the Poisson regime of small E)
        assert fig["far"] == 0, describe(what, fig)
        assert fig["mism"] <= fig["cap"], describe(what, fig)
    if "emu_mism" in fig:
        # (c) the same expression evaluated twice in fp32: E32 = sum min(1, 2 arith32 / step) values may round differently, by one step
        assert fig["emu_far"] == 0, describe(what, fig)
        assert fig["emu_mism"] <= fig["cap32"], describe(what, fig)
    return fig
