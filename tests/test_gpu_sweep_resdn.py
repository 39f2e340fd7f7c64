"""-m gpu: every finite 16-bit value through prelu_kernel (ResDN's per-channel PReLU, esr_prelu) and resdb_step_kernel (its one-launch step, esr_resdb_step) -- through its activation and its store -- with
the helpers and comparators of tests/test_gpu_value_sweep.py (DESIGN.md "Value sweep").

It lives in a file of its own and ENTERS ITSELF into that module's registry when this file is imported, as tests/test_gpu_sweep_arfdn.py
does: `SWEPT` gets the kernel, and the test function becomes an attribute of that module, which is where
tests/test_sweep_helper.py::test_every_kernel_is_swept_or_exempt looks for it."""
import pytest
import torch

import _resdn as R
import _sweep as S
import test_gpu_value_sweep as V
from test_gpu_value_sweep import DEV, STORES, _report, _sweep, _traced

pytestmark = pytest.mark.gpu
C = 32
# a negative slope, one in (0, 1) and one above 1 whose significands are short (the product is exact or an exact tie in many places), and the
# checkpoint's extremes as fp32 numbers with full significands (the product needs its ONE rounding: fp64 -> fp32 -> 16-bit would round twice)
SLOPES = (-1.5, 0.25, 2.5, -1.82, 0.3, 3.62)


@pytest.mark.parametrize("store", STORES)
def test_prelu(store):
    """prelu_kernel on the tiled sweep, one slope for all channels per launch: a non-negative value comes back bit for bit (-0 included), a
    negative one as the exact product a v rounded once to nearest even -- subnormal results and overflow to Inf included; the kernel has no
    matrix product, so no subnormal input is exempt."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    S.assert_exempt_share(_sweep(store))
    n, h, w = S.shape_for(_sweep(store), C)
    x = S.tile(_sweep(store), (n, h, w, C))
    xd = x.to(DEV)
    for slope in SLOPES:
        a = torch.full((C,), slope, dtype=torch.float32)
        y, name = _traced(rf"prelu_kernel<{1 if store == 'bf16' else 2}, true>", lambda: ops.prelu([xd], a))
        want = R.prelu_stored(x, a)
        label = f"prelu {store} slope {slope} {n}x{h}x{w}"
        took = S.exact(y.cpu(), want, dt, v=x.float(), what=label)
        keep = x.float() >= 0
        assert torch.equal(S.to_bits(y.cpu())[keep], S.to_bits(x)[keep]), label + ": a non-negative value passes through bit for bit"
        assert took == 0
        _report(label, name, took)


@pytest.mark.parametrize("store", STORES)
def test_resdb_step(store):
    """resdb_step_kernel with 0 / 1 weights, so every stage is exact.  `d`: the distilled rows select x, dists = (prelu(x, a_e))~ -- u is an MFMA
    operand, a subnormal one may be read as zero; `x`: all weights zero, y = x through the residual; `t`: a_e = 1, the `res` rows select x, the
    3x3 is a centre-tap identity, y = (x + (prelu(x, a_c))~)~ with a_c = -0.75 (the sum is exact in fp32; where x or t is subnormal the matrix
    core may read it as zero: y = x).  Slopes of magnitude at most 1 here: a product that overflows to Inf would meet the zero weights of the
    pixel's other channels (0 x Inf); slopes above 1 over every value are test_prelu's, and over random data tests/test_gpu_resdn.py's."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n_exempt = S.assert_exempt_share(_sweep(store))
    n, h, w = S.shape_for(_sweep(store), 48)
    x = S.tile(_sweep(store), (n, h, w, 48))
    xd = x.to(DEV)
    sel = torch.zeros(96, 48)
    sel[torch.arange(96), torch.arange(96) % 48] = 1.0
    res_only, dist_only = sel.clone(), sel.clone()
    res_only[48:] = 0
    dist_only[:48] = 0
    eye3 = S.identity_weight(48, 48, 3)
    z96, z48, one = torch.zeros(96), torch.zeros(48), torch.ones(48)
    kern = rf"resdb_step_kernel<{'true' if store == 'bf16' else 'false'}, 0, 3>"
    sub = S.is_subnormal
    for slope in (-0.75, 0.25, 1.0):
        a = torch.full((48,), slope)
        (dd, y), name = _traced(kern, lambda: ops.resdb_step(xd, a, dist_only, z96, one, torch.zeros(48, 48, 3, 3), z48))
        u = R.prelu_stored(x, a)
        took = S.exact(dd.cpu(), u, dt, v=x.float(), flushed=torch.where(sub(u), torch.zeros_like(u), u), what=f"resdb step {store} d slope {slope}")
        took += S.exact(y.cpu(), x, dt, v=x.float(), what=f"resdb step {store} x")
        _report(f"resdb step {store} terms d, x slope {slope} {n}x{h}x{w}", name, took, 2 * n_exempt)
    a = torch.full((48,), -0.75)
    (dd, y), name = _traced(kern, lambda: ops.resdb_step(xd, one, res_only, z96, a, eye3, z48))
    t = R.prelu_stored(x, a)
    want = R.store_once(x.double() + t.double(), dt)
    took = S.exact(y.cpu(), want, dt, v=x.float(), flushed=torch.where(sub(x) | sub(t), x, want), what=f"resdb step {store} t")
    _report(f"resdb step {store} term t {n}x{h}x{w}", name, took, int((sub(x) | sub(t)).sum()))


def _listed(fn):
    """a case of this file as the registry module names it: callable(store) runs the case.  A class, because pytest collects a module's
    test_* FUNCTIONS (the cases would run a second time from that module) and warns about any other callable of that name but a class"""
    return type(fn.__name__, (), {"__new__": lambda cls, *args, **kw: fn(*args, **kw), "__doc__": fn.__doc__})


V.SWEPT.update({"prelu_kernel": ["test_prelu"], "resdb_step_kernel": ["test_resdb_step"]})
V.test_prelu = _listed(test_prelu)
V.test_resdb_step = _listed(test_resdb_step)
