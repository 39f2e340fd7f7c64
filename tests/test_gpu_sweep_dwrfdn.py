"""-m gpu: every finite 16-bit value through the two kernels of team 35's RFDN, dwpw_pair_kernel and esa_unshuffle_kernel -- the cases of
tests/test_gpu_value_sweep.py for them, with that module's helpers and comparators (DESIGN.md "Value sweep").

They live in a file of their own and ENTER THEMSELVES into that module's registry when this file is imported: `SWEPT` gets the two
kernels, and the two test functions become attributes of that module, which is where tests/test_sweep_helper.py::
test_every_kernel_is_swept_or_exempt looks for them.  pytest imports every test file of a run before it runs a test, so the closure test
sees the entries whenever the suite (or this file together with tests/test_sweep_helper.py) is collected; run on its own,
tests/test_sweep_helper.py reports the two kernels as missing."""
import pytest
import torch

import _sweep as S
import test_gpu_value_sweep as V
from test_gpu_value_sweep import DEV, LRELU, RELU, RES_PRE, SLOPE, STORES, _bf, _expr, _flush, _report, _stage, _sweep, _traced

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("store", STORES)
def test_dwpw_pair(store):
    """dwpw_pair_kernel: u1 = dw_a(x) + x, h = relu(S . u1), u2 = dw_b(h) + h, out = lrelu(S' . u2 + x).  Every weight zero: out = lrelu(x),
    the residual route, nothing exempt.  Identity 1x1s and zero depthwise layers: out = lrelu(relu(x) + x), one fp32 add, one rounding.
    The two hidden stores that round a VALU sum, u1 and u2: a centre tap of 1/4 makes them rnd(1.25 v) -- a tie for every fourth value --
    and they are handed out exactly through channels where x is zero (0 / 1 weights, slope 1: nothing is rounded again); the few values
    whose 1.25-fold overflows the storage type are left to the first two routes."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    c = 48
    n, h, w = 2, 23, 37
    pat = rf"dwpw_pair_kernel<{_bf(store)}>"
    x = S.tile(_sweep(store), (n, h, w, c))
    xd = x.to(DEV)
    z3, zb, eye, zero = torch.zeros(c, 1, 3, 3), torch.zeros(c), torch.eye(c), torch.zeros(c, c)
    y, name = _traced(pat, lambda: ops.dwpw_pair(xd, z3, zb, zero, zb, z3, zb, zero, zb, slope=SLOPE))
    want, skip = _expr(torch.zeros(n, h, w, c), x.float(), LRELU, RES_PRE, dt)
    label = f"dwpw pair {store} all weights zero {n}x{h}x{w}"
    S.exact(torch.where(skip, want, y.cpu()[..., :c]), want, dt, v=x.float(), what=label)
    _report(label, name, 0)
    y, name = _traced(pat, lambda: ops.dwpw_pair(xd, z3, zb, eye, zb, z3, zb, eye, zb, slope=SLOPE))
    refs = []
    for flush in (False, True):
        h16, _ = _stage(x, RELU, flush)
        refs.append(_expr((_flush(h16) if flush else h16).float(), x.float(), LRELU, RES_PRE, dt))
    (want, skip), (alt, _) = refs
    label = f"dwpw pair {store} identity 1x1s {n}x{h}x{w}"
    took = S.exact(torch.where(skip, want, y.cpu()[..., :c]), want, dt, v=x.float(), flushed=alt, what=label)
    _report(label, name, took, int(S.is_subnormal(x).sum()))
    # the hidden stores: the sweep on channels 0 .. 23, x = 0 on 24 .. 47, where the results come out
    half = c // 2
    n, h, w = S.shape_for(_sweep(store), half)
    x = S.tile(_sweep(store), (n, h, w, c), half)
    x = torch.where(torch.isfinite((x.float() * 1.25).to(dt)), x, torch.zeros_like(x))
    xd = x.to(DEV)
    quarter = 0.25 * S.dw_identity(c, 3)
    quarter[half:] = 0
    route, keep, first = torch.zeros(c, c), torch.zeros(c, c), torch.zeros(c, c)
    for j in range(half):
        route[half + j, j] = keep[half + j, half + j] = first[j, j] = 1.0
    xl = x[..., :half]
    # u1 = rnd(1.25 x), through the ReLU as relu(u1) - relu(-u1)
    pos, name = _traced(pat, lambda: ops.dwpw_pair(xd, quarter, zb, route, zb, z3, zb, keep, zb, slope=1.0))
    neg = ops.dwpw_pair(xd, quarter, zb, -route, zb, z3, zb, keep, zb, slope=1.0)
    torch.cuda.synchronize()
    got = (pos.cpu()[..., half:c].float() - neg.cpu()[..., half:c].float()).to(dt)
    want = (xl.float() * 0.25 + xl.float()).to(dt)
    label = f"dwpw pair {store} u1 = 1.25 x {n}x{h}x{w}"
    took = S.exact(got, want, dt, v=xl.float(), flushed=_flush(want), what=label)
    _report(label, name, took, int(S.is_subnormal(want).sum()))
    # u2 = rnd(1.25 h), h = relu(x)
    y, name = _traced(pat, lambda: ops.dwpw_pair(xd, z3, zb, first, zb, quarter, zb, route, zb, slope=1.0))
    refs = []
    for flush in (False, True):
        h16, _ = _stage(xl, RELU, flush)
        u2 = (h16.float() * 0.25 + h16.float()).to(dt)
        refs.append(_flush(u2) if flush else u2)
    want, alt = refs
    label = f"dwpw pair {store} u2 = 1.25 relu(x) {n}x{h}x{w}"
    took = S.exact(y.cpu()[..., half:c], want, dt, v=xl.float(), flushed=alt, what=label)
    _report(label, name, took, int(S.is_subnormal(xl).sum() + S.is_subnormal(want).sum()))
    ties = int(((xl.float() * 1.25).double() - want.double() != 0).sum())
    assert ties > xl.numel() // 8, ties                            # (the 1.25-fold needs a rounding for a large share of the values)


@pytest.mark.parametrize("store", STORES + ["f32"])
def test_esa_unshuffle(store):
    """esa_unshuffle_kernel: the conv1 map of image i holds ONE 16-bit value per channel at every pixel of its 14 x 14 pixels, so the pooled
    pixel is that value; con_ selects unshuffled channel 4 o: c3 = relu(relu(v)), exactly, in fp32 -- a load that converts wrongly, a
    maximum or an activation that changes a value shows.  f32: the bf16 patterns widened."""
    from ntire2022_esr_amd import ops
    sw = _sweep("bf16" if store == "f32" else store)
    f = 16
    n = -(-sw.numel() // f)
    v = torch.zeros(n * f, dtype=sw.dtype)
    v[:sw.numel()] = sw
    c1 = v.view(n, 1, 1, f).expand(n, 14, 14, f).contiguous()
    if store == "f32":
        c1 = c1.float()
    wt = torch.zeros(f, 4 * f, 1, 1)
    for o in range(f):
        wt[o, 4 * o + (o & 3)] = 1.0                              # (every one of the four sub-pixel positions is selected by some channel)
    y, name = _traced(rf"esa_unshuffle_kernel<{ {'f32': 0, 'bf16': 1, 'f16': 2}[store] }>", lambda: ops.esa_unshuffle(c1.to(DEV), wt, torch.zeros(f)))
    y = y.cpu()
    assert y.dtype == torch.float32 and tuple(y.shape) == (n, 3, 3, 16)
    want = torch.fmax(v.float(), torch.zeros(())).view(n, f)
    bad = ~(y[:, 1, 1, :].double() == want.double())
    assert not bool(bad.any()), (int(bad.sum()), float(v.view(n, f)[bad][0]))
    ring = y.clone()
    ring[:, 1, 1, :] = 0
    assert not bool(ring.any())                                    # relu(bias = 0) around the one pooled pixel
    print(f"esa unshuffle {store}: {name}; {sw.numel()} values, all exact")


def _listed(fn):
    """a case of this file as the registry module names it: callable(store) runs the case.  A class, because pytest collects a module's
    test_* FUNCTIONS (the cases would run a second time from that module) and warns about any other callable of that name but a class"""
    return type(fn.__name__, (), {"__new__": lambda cls, *args, **kw: fn(*args, **kw), "__doc__": fn.__doc__})


V.SWEPT.update({"dwpw_pair_kernel": ["test_dwpw_pair"], "esa_unshuffle_kernel": ["test_esa_unshuffle"]})
V.test_dwpw_pair, V.test_esa_unshuffle = _listed(test_dwpw_pair), _listed(test_esa_unshuffle)
