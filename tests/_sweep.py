"""Every 16-bit value through a kernel's activation and store (tests/test_gpu_value_sweep.py; DESIGN.md "Value sweep").

The fp64 cases of the suite draw randn inputs and grant "half a storage step x 1.01 plus a slack": they see the accumulation, not the
rounding of an exact tie, not an activation outside |v| < 5, not a drift between the copies of the 16-bit GELU polynomial and of the
sigmoid.  A 16-bit type has 65 536 values: all finite ones fit in one 1 x 32 x 32 x 64 tensor, and with weights that are only 0 and 1
the pre-activation v of a convolution is EXACT -- v is the swept value itself, either as the residual of a zero convolution (the
residual route) or as the input of an identity convolution (the identity route).  The reference then needs no accumulation tolerance.

This module is the CPU side: the sweeps, the tie pairs, the 0 / 1 weights, the emulation of the polynomial, the comparators, and emulated
WRONG stores / activations that the comparators must reject (tests/test_sweep_helper.py runs all of it without a GPU)."""
import math

import numpy as np
import torch

DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
MBITS = {torch.bfloat16: 7, torch.float16: 10}                     # stored significand bits
EMIN = {torch.bfloat16: -126, torch.float16: -14}                  # exponent of the smallest normal
N_FINITE = {torch.bfloat16: 65280, torch.float16: 63488}
N_SUBNORMAL = {torch.bfloat16: 254, torch.float16: 2046}           # non-zero subnormal patterns: the identity route's flush exemption
F32_MIN_NORMAL = 2.0 ** -126
ROW_OFFSET = 5                                                     # tile(): a row starts this many values before the previous row's end


# ---- bit patterns ---------------------------------------------------------------------------------------------------------------------
def from_bits(bits, dt):
    """int tensor of 16-bit patterns (0 .. 65535) -> tensor of dt"""
    b = bits.to(torch.int32)
    return (b - 65536 * (b >= 32768).to(torch.int32)).to(torch.int16).view(dt)


def to_bits(t):
    """16-bit float tensor -> int32 patterns 0 .. 65535"""
    return t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


def all_finite(dt):
    """every finite bit pattern of dt in pattern order (+0, the positive subnormals and normals, -0, the negative ones)"""
    v = from_bits(torch.arange(65536), dt)
    v = v[torch.isfinite(v.float())].clone()
    assert v.numel() == N_FINITE[dt], v.numel()
    return v


def is_subnormal(t):
    """non-zero and below the smallest normal of t's own type"""
    a = t.double().abs()
    return (a > 0) & (a < 2.0 ** EMIN[t.dtype])


def permuted(sweep, mult=24593, add=12289):
    """a second fixed ordering of a sweep: value i of the result is sweep[(i * mult + add) mod len] (mult is coprime to both lengths)"""
    n = sweep.numel()
    assert math.gcd(mult, n) == 1, (mult, n)
    return sweep[(torch.arange(n, dtype=torch.int64) * mult + add) % n].clone()


def tile(values, shape, channels=None):
    """an [N, H, W, C] tensor of values.dtype whose first `channels` channels (default: all C; the others are zeros) hold `values` in order,
    repeated to the end; each image row starts ROW_OFFSET values before the point where the previous row stopped, so that a repetition of
    the sweep does not put a value into the lane and channel position it had before.  Asserts that every value is in the tensor."""
    n, h, w, c = shape
    cl = c if channels is None else channels
    rows, rowlen = n * h, w * cl
    off = ROW_OFFSET if rowlen > ROW_OFFSET else 0
    idx = (torch.arange(rows, dtype=torch.int64)[:, None] * (rowlen - off) + torch.arange(rowlen, dtype=torch.int64)[None, :])
    assert int(idx.max()) + 1 >= values.numel(), f"{tuple(shape)} x {cl} channels holds {int(idx.max()) + 1} of {values.numel()} values"
    core = values[idx % values.numel()].reshape(n, h, w, cl)
    out = torch.zeros(n, h, w, c, dtype=values.dtype)
    out[..., :cl] = core
    return out


def shape_for(values, channels, w=37, n=2):
    """the smallest [n, H, w] with H odd and >= 23 whose `channels` channels hold all of `values` (ragged against 16-pixel tiles)"""
    rowlen = w * channels - ROW_OFFSET
    h = max(23, -(-(values.numel() + ROW_OFFSET) // (n * rowlen)))
    return n, h + (1 - h % 2), w


# ---- neighbours in the storage type, and stores that are NOT round-to-nearest-even ----------------------------------------------------------
def _step_up(t):
    """the next value of t's type towards +inf (finite t)"""
    b = to_bits(t)
    b = torch.where(b == 0x8000, torch.zeros_like(b), b)                                   # -0 counts as +0
    return from_bits(torch.where(b < 0x8000, b + 1, b - 1), t.dtype)


def _step_down(t):
    b = to_bits(t)
    b = torch.where(b == 0, torch.full_like(b, 0x8000), b)
    return from_bits(torch.where(b >= 0x8000, b + 1, b - 1), t.dtype)


def neighbours(s, dt):
    """the values lo <= s <= hi of dt that bracket the fp64 tensor s (lo == hi where s is a value of dt; +-inf beyond the range)"""
    r = s.to(dt)                                                                           # round-to-nearest-even
    rd = r.double()
    big = torch.isinf(rd)
    top = torch.full_like(r, torch.finfo(dt).max)
    lo = torch.where(rd <= s, r, torch.where(big, top, _step_down(torch.where(big, top, r))))
    hi = torch.where(rd >= s, r, torch.where(big, -top, _step_up(torch.where(big, -top, r))))
    return lo, hi


def store_rne(s, dt):
    """the store every kernel is to perform: fp32 -> dt, round to nearest, ties to even"""
    return s.float().to(dt)


def store_ties_away(s, dt):
    """a WRONG store: round to nearest, ties away from zero (what adding half a step to the magnitude and truncating gives)"""
    s = s.double()
    lo, hi = neighbours(s, dt)
    tie = (s - lo.double() == hi.double() - s) & (lo.double() != hi.double()) & torch.isfinite(lo.double()) & torch.isfinite(hi.double())
    return torch.where(tie, torch.where(s < 0, lo, hi), s.to(dt))


def store_truncate(s, dt):
    """a WRONG store: the low bits dropped (round towards zero)"""
    s = s.double()
    lo, hi = neighbours(s, dt)
    return torch.where(s < 0, hi, lo)


# ---- tie pairs ------------------------------------------------------------------------------------------------------------------------------
def tie_pairs(dt):
    """(x, r, info): x over all normal finite values of dt, r = +-1/2, +-1/4, +-3/4 of x's storage step wherever that is a value of dt (it
    is not for the lowest two binades); x + r is exact in fp32 -- an exact tie for half a step (unless x is a power of two and r points
    towards zero), just to either side of one otherwise.  info counts the ties by the side of their even neighbour."""
    sw = all_finite(dt)
    x = sw[~is_subnormal(sw) & (sw.float() != 0)]
    xd = x.double()
    step = torch.exp2(torch.floor(torch.log2(xd.abs())) - MBITS[dt])
    xs, rs = [], []
    for f in (0.5, -0.5, 0.25, -0.25, 0.75, -0.75):
        r = step * f
        ok = r.to(dt).double() == r
        xs.append(x[ok])
        rs.append(r[ok].to(dt))
    x, r = torch.cat(xs), torch.cat(rs)
    s = x.double() + r.double()
    assert bool((s.float().double() == s).all()), "x + r must be exact in fp32"
    lo, hi = neighbours(s, dt)
    tie = (s - lo.double() == hi.double() - s) & (lo.double() != hi.double())
    fin = torch.isfinite(hi.double()) & torch.isfinite(lo.double())
    even_lo = tie & fin & (to_bits(lo) % 2 == 0)
    even_hi = tie & fin & (to_bits(hi) % 2 == 0)
    # beyond the largest finite value the "even neighbour" is the power of two the format cannot hold: the conversion gives Inf
    to_inf = torch.isinf((x.float() + r.float()).to(dt).float())
    info = {"pairs": x.numel(), "ties": int(tie.sum()), "even_below": int(even_lo.sum()), "even_above": int(even_hi.sum()), "to_inf": int(to_inf.sum())}
    assert info["even_below"] >= 30000 and info["even_above"] >= 30000, info
    assert not bool((even_lo & even_hi).any())
    if dt == torch.float16:
        assert info["to_inf"] >= 2 and bool((x.float().abs()[to_inf] == 65504.0).all()), info       # +-65504 +- 16 -> +-Inf
    return x, r, info


# ---- weights that are only 0 and 1 ---------------------------------------------------------------------------------------------------------
def zero_weight(cout, cin, k):
    return torch.zeros(cout, cin, k, k)


def identity_weight(cout, cin, k=3):
    """centre-tap identity / selection: output channel o <- input channel o mod cin (a 0 / 1 selection matrix for unequal widths)"""
    w = torch.zeros(cout, cin, k, k)
    o = torch.arange(cout)
    w[o, o % cin, k // 2, k // 2] = 1.0
    return w


def selection(cout, cin):
    """identity_weight as the [cout, cin] matrix of a 1x1"""
    return identity_weight(cout, cin, 1)[:, :, 0, 0].contiguous()


def dw_identity(c, k):
    """depthwise [c, 1, k, k]: centre tap 1"""
    w = torch.zeros(c, 1, k, k)
    w[:, 0, k // 2, k // 2] = 1.0
    return w


def blob_words(blob, dt):
    """a packed weight blob as 16-bit words of dt (the images of a 16-bit packer; its fp32 biases show as pairs of words)"""
    return blob.detach().cpu().contiguous().view(torch.uint8).view(dt)


def assert_blob_is_0_1(blob, dt, ones, what):
    """For the packers that have no unpacking entry point (post, tail, apply-post): every 16-bit word of a blob packed from 0 / 1 matrices
    with zero biases must be +0 or the type's 1.0 -- no low part, no diffused error, no rounding residue --, and the 1.0 words must be
    whole images (1 .. 8 of each) of the matrices' `ones` counts (an int, or one int per matrix).  WHERE the ones sit is what the GPU cases
    check.  Returns the number of 1.0 words."""
    ones = [ones] if isinstance(ones, int) else list(ones)
    b = to_bits(blob_words(blob, dt))
    one = int(to_bits(torch.ones(1, dtype=dt))[0])
    other = (b != 0) & (b != one)
    assert not bool(other.any()), (what, "words other than 0 and 1.0", [hex(int(v)) for v in b[other][:8]])
    n1 = int((b == one).sum())
    sums = {0}
    for o in ones:
        sums = {s + k * o for s in sums for k in range(1, 9)}
    assert n1 in sums, (what, f"{n1} words of 1.0 for matrices of {ones} ones")
    return n1


# ---- the 16-bit GELU polynomial, emulated ---------------------------------------------------------------------------------------------------
GELU16_COEFFS = (-1.580786198e-09, 1.217111051e-07, -4.100866386e-06, 8.066739505e-05, -1.048204400e-03, 9.664874174e-03,
                 -6.617537882e-02, 3.988475079e-01)
GELU16_CLAMP = 4.0
# |gelu16 - GELU|, from gelu16_cpu over every finite bf16 and f16 value (tests/test_sweep_helper.py prints and asserts the three pieces):
GELU16_BOUND_BELOW = 2.13e-4          # v < -4: the function is the constant -4 * (0.5 - 4 P(16)) = -2.127e-4 while GELU(v) -> 0
GELU16_BOUND_MID = 1.3e-4             # -4 <= v <= 4 (documented; the emulation gives 8.8e-5)
GELU16_BOUND_SLOPE = 5.33e-5          # v > 4: this times v (x * (1 - Phi_poly(4)) = 5.3225e-5 x against x * (1 - Phi(x)) -> 0; documented to two digits: 5.3e-5)
GELU16_DOC_SLOPE = 5.3e-5


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product is exact in fp64, the sum is rounded once to fp64 and then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gelu16_cpu(v, coeffs=GELU16_COEFFS, clamp=GELU16_CLAMP, clamp_factor=None):
    """gelu16 (esr_s16_dev.h) on an fp32 / 16-bit tensor -> fp32 tensor: xc = med3(x, -clamp, clamp), t = xc * xc, Horner in fp32 with one
    rounding per fmaf, max(x, -clamp) * fma(xc, p, 0.5).  `coeffs` / `clamp` other than the defaults emulate a drifted copy."""
    x = v.detach().float().numpy().astype(np.float32)
    c32 = [np.float32(c) for c in coeffs]
    cl = np.float32(clamp)
    xc = np.minimum(np.maximum(x, -cl), cl)
    t = (xc.astype(np.float64) * xc.astype(np.float64)).astype(np.float32)
    p = np.full_like(x, c32[0])
    for c in c32[1:]:
        p = _fma32(p, t, np.full_like(x, c))
    q = _fma32(xc, p, np.full_like(x, np.float32(0.5)))
    y = (np.maximum(x, -cl).astype(np.float64) * q.astype(np.float64)).astype(np.float32)
    return torch.from_numpy(y)


def gelu_f64(v):
    return torch.nn.functional.gelu(v.double())


def gelu16_bound(v):
    """B(v): the piecewise bound of |gelu16(v) - GELU(v)| as an fp64 tensor"""
    v = v.double()
    return torch.where(v < -4.0, torch.full_like(v, GELU16_BOUND_BELOW),
                       torch.where(v > 4.0, GELU16_BOUND_SLOPE * v, torch.full_like(v, GELU16_BOUND_MID)))


def gelu16_error_pieces(sweeps):
    """(max |gelu16_cpu - GELU| on v < -4, the same on [-4, 4], max of it / v on v > 4) over the given sweeps"""
    lo = mid = slope = 0.0
    for sw in sweeps:
        v = sw.double()
        err = (gelu16_cpu(sw).double() - gelu_f64(sw)).abs()
        lo = max(lo, float(err[v < -4].max()))
        mid = max(mid, float(err[(v >= -4) & (v <= 4)].max()))
        slope = max(slope, float((err[v > 4] / v[v > 4]).max()))
    return lo, mid, slope


def sigmoid_f64(v):
    """1 / (1 + exp(-v)) in fp64, as exp(v) / (1 + exp(v)) for v < 0 (no overflow, full relative accuracy down to the smallest results)"""
    v = v.double()
    e = torch.exp(-v.abs())
    return torch.where(v < 0, e / (1.0 + e), 1.0 / (1.0 + e))


def sigmoid_tanh_f16(v):
    """a WRONG sigmoid: 0.5 * (1 + tanh(v / 2)) with every operation rounded to fp16 -> fp32 tensor"""
    h = (v.float() * 0.5).half()
    t = torch.tanh(h.float()).half()
    return ((1.0 + t.float()).half().float() * 0.5).half().float()


# ---- tolerances -------------------------------------------------------------------------------------------------------------------------------
def half_step(ref, dt):
    """half the distance between the neighbours of dt around the fp64 tensor ref (the subnormal step below the smallest normal): what one
    correct rounding of ref may cost"""
    a = ref.double().abs()
    e = torch.floor(torch.log2(torch.clamp(a, min=2.0 ** EMIN[dt])))
    return torch.exp2(e - MBITS[dt] - 1)


def store_tol(ref, dt):
    """half a storage step x 1.01"""
    return half_step(ref, dt) * 1.01


def f32_tol(ref):
    """fp32 storage: 4 * 2^-24 * |ref|, and never less than half the smallest fp32 subnormal (2^-150): below 2^-126 the format's step is
    2^-149 whatever the value, and a correct result of 1e-46 is stored as 0"""
    return ref.double().abs() * (4 * 2.0 ** -24) + 2.0 ** -150


# ---- comparators --------------------------------------------------------------------------------------------------------------------------------
class Mismatch(AssertionError):
    pass


def _worst(what, bad, score, v, got, want):
    i = int(torch.argmax(torch.where(bad, score, torch.full_like(score, -1.0)).reshape(-1)))
    pos = tuple(int(p) for p in np.unravel_index(i, tuple(got.shape)))
    vv = "" if v is None else f"v = {float(v.reshape(-1)[i]):.9g}, "
    return f"{what}: {int(bad.sum())} of {bad.numel()} wrong; worst: {vv}position {pos}, got {float(got.reshape(-1)[i]):.9g}, want {float(want.reshape(-1)[i]):.9g}"


def exact(got, want, dt, v=None, flushed=None, what="exact"):
    """got == want as values of dt: +0 equals -0, an Inf must stand where want has one (same sign), no NaN.  `flushed`: the reference
    computed with the exempt inputs (flush_mask: subnormal MFMA operands of the identity route) read as zero -- it differs from `want`
    at those positions only, and there, and only there, got may equal it instead (with nothing but the swept input in v: +-0).  `v`: the
    swept value per position, for the message.  Prints the worst case and raises Mismatch; returns how many positions took `flushed`."""
    assert got.dtype == dt and want.dtype == dt and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    bad = ~(g == w)                                                                        # NaN on either side: unequal
    took = 0
    if flushed is not None:
        f = flushed.detach().cpu().double()
        took = int((bad & (g == f)).sum())
        bad &= ~(g == f)
    if bool(bad.any()):
        score = torch.nan_to_num((g - w).abs(), nan=float("inf"), posinf=float("inf"))
        msg = _worst(what, bad, score, v, g, w)
        print(msg)
        raise Mismatch(msg)
    return took


def within(got, ref, tol, v=None, what="within"):
    """|got - ref| <= tol elementwise in fp64 (a non-finite got fails).  Returns the largest |got - ref| and |got - ref| / tol; prints
    the worst case and raises Mismatch."""
    g, r, t = got.detach().cpu().double(), ref.detach().cpu().double(), tol.detach().cpu().double()
    assert g.shape == r.shape and t.shape == r.shape, (g.shape, r.shape, t.shape)
    d = (g - r).abs()
    bad = ~(d <= t)
    if bool(bad.any()):
        score = torch.nan_to_num(d / torch.clamp(t, min=1e-300), nan=float("inf"), posinf=float("inf"))
        msg = _worst(what, bad, score, v, g, r)
        print(msg)
        raise Mismatch(msg)
    ratio = d / torch.clamp(t, min=1e-300)
    return float(d.max()), float(ratio.max())


def flush_mask(x):
    """the identity route's only exemption: positions whose swept INPUT is subnormal in its storage type (an MFMA operand: the matrix core
    may read it as zero)"""
    return is_subnormal(x)


def assert_exempt_share(values):
    """254 of 65 280 bf16 patterns / 2 046 of 63 488 f16 patterns are exempt on the identity route, nothing else"""
    dt = values.dtype
    m = flush_mask(values)
    assert values.numel() == N_FINITE[dt] and int(m.sum()) == N_SUBNORMAL[dt], (values.numel(), int(m.sum()))
    return int(m.sum())
