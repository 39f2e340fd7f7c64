"""-m gpu: every finite 16-bit value through conv_prelu_kernel's epilogue (MDGN's 3x3 + PReLU, esr_conv_prelu) and through mdsa_gate_kernel (the
end of its block, esr_mdsa_gate) with the helpers and comparators of tests/test_gpu_value_sweep.py (DESIGN.md "Value sweep").

It lives in a file of its own and ENTERS ITSELF into that module's registry when this file is imported, as tests/test_gpu_sweep_resdn.py
does: `SWEPT` gets the kernels, and the test functions become attributes of that module, which is where
tests/test_sweep_helper.py::test_every_kernel_is_swept_or_exempt looks for them."""
import pytest
import torch

import _mdgn as M
import _resdn as R
import _sweep as S
import test_gpu_value_sweep as V
from test_gpu_value_sweep import DEV, STORES, _report, _sweep, _traced

pytestmark = pytest.mark.gpu
C = 64
# the checkpoint's extremes, a value in (0, 1), the identity, ResDN's largest slope (above 1: nn.PReLU allows it) as fp32 numbers with full
# significands -- the product needs its ONE rounding: fp64 -> fp32 -> 16-bit would round twice -- and 0
SLOPES = (-0.88, 0.25, 1.0, 3.62, 0.0)


@pytest.mark.parametrize("store", STORES)
def test_conv_prelu_epilogue(store):
    """conv_prelu_kernel with an identity centre tap and zero bias: the accumulator IS the swept value (a subnormal one is an MFMA operand and
    may be read as zero), one slope for all channels per launch.  A positive value comes back bit for bit, a negative one as the exact
    product a v rounded once to nearest even -- ties, subnormal results and overflow to Inf included (tests/_sweep.py's method)."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n_exempt = S.assert_exempt_share(_sweep(store))
    n, h, w = S.shape_for(_sweep(store), C)
    x = S.tile(_sweep(store), (n, h, w, C))
    xd = x.to(DEV)
    eye3, zero = S.identity_weight(C, C, 3), torch.zeros(C)
    sub = S.is_subnormal(x)
    for slope in SLOPES:
        a = torch.full((C,), slope, dtype=torch.float32)
        y, name = _traced(rf"conv_prelu_kernel<{'true' if store == 'bf16' else 'false'}>", lambda: ops.conv_prelu(xd, eye3, zero, a))
        want = R.prelu_stored(x, a)
        label = f"conv_prelu {store} slope {slope} {n}x{h}x{w}"
        took = S.exact(y.cpu(), want, dt, v=x.float(), flushed=torch.where(sub, torch.zeros_like(want), want), what=label)
        keep = (x.float() > 0) & ~sub                      # (a zero comes back as +0: the accumulator is a sum)
        assert torch.equal(S.to_bits(y.cpu())[keep], S.to_bits(x)[keep]), label + ": a positive value passes through bit for bit"
        _report(label, name, took, n_exempt)


@pytest.mark.parametrize("store", STORES)
def test_mdsa_gate(store):
    """mdsa_gate_kernel with W_f selecting f1, b_f = 0 and a closed gate argument (w_s = 0, b_s = 0: s = 1/2 exactly): y = store(prelu(v, a) / 2),
    the PReLU's product and the halving as the fp32 operations the header says they are.  The slopes have short significands, so the fp32
    product is exact -- or, for 2.5 times the largest bf16 values, Inf, as in the reference's fp32 -- and the store is the only rounding."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n_exempt = S.assert_exempt_share(_sweep(store))
    n, h, w = S.shape_for(_sweep(store), C)
    x = S.tile(_sweep(store), (n, h, w, C))
    f = torch.zeros(n, h, w, 3 * C, dtype=dt)
    f[..., :C] = x
    fd, xd = f.to(DEV), torch.zeros(n, h, w, C, dtype=dt, device=DEV)
    w_f = torch.zeros(C, 3 * C)
    w_f[torch.arange(C), torch.arange(C)] = 1.0
    zero = torch.zeros(C)
    sub = S.is_subnormal(x)
    for slope in (-0.75, 0.25, 1.0, 2.5):
        a = torch.full((C,), slope, dtype=torch.float32)
        y, name = _traced(rf"mdsa_gate_kernel<{'true' if store == 'bf16' else 'false'}>", lambda: ops.mdsa_gate(fd, xd, w_f, zero, a, zero, torch.zeros(1)))
        f32 = torch.where(x.float() >= 0, x.float(), a * x.float())                         # fp32, exact wherever it does not overflow
        assert bool(((f32.double() == R.prelu_f64(x.double(), a)) | torch.isinf(f32)).all())
        want = R.store_once((f32 * 0.5).double(), dt)
        label = f"mdsa_gate {store} slope {slope} {n}x{h}x{w}"
        took = S.exact(y.cpu(), want, dt, v=x.float(), flushed=torch.where(sub, torch.zeros_like(want), want), what=label)
        _report(label, name, took, n_exempt)


def _listed(fn):
    """a case of this file as the registry module names it: callable(store) runs the case.  A class, because pytest collects a module's
    test_* FUNCTIONS (the cases would run a second time from that module) and warns about any other callable of that name but a class"""
    return type(fn.__name__, (), {"__new__": lambda cls, *args, **kw: fn(*args, **kw), "__doc__": fn.__doc__})


V.SWEPT.update({"conv_prelu_kernel": ["test_conv_prelu_epilogue"], "mdsa_gate_kernel": ["test_mdsa_gate"]})
V.test_conv_prelu_epilogue = _listed(test_conv_prelu_epilogue)
V.test_mdsa_gate = _listed(test_mdsa_gate)
