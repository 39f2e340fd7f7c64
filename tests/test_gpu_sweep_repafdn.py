"""-m gpu: every finite 16-bit value through the two kernels of RePAFDN's tail, pa_gate_kernel and pa_tail_kernel -- through their sigmoid,
their product and their store -- with the helpers and comparators of tests/test_gpu_value_sweep.py (DESIGN.md "Value sweep").

They live in a file of their own and ENTER THEMSELVES into that module's registry when this file is imported, as
tests/test_gpu_sweep_dwrfdn.py does: `SWEPT` gets the two kernels, and the two test functions become attributes of that module, which is
where tests/test_sweep_helper.py::test_every_kernel_is_swept_or_exempt looks for them."""
import pytest
import torch

import _sweep as S
import test_gpu_value_sweep as V
from test_gpu_value_sweep import DEV, STORES, _bf, _flush, _perm, _report, _sweep, _traced

pytestmark = pytest.mark.gpu
C = 48
NHW = (2, 23, 37)


def _zero_gate(bias):
    return torch.zeros(C, C), torch.full((C,), float(bias))


@pytest.mark.parametrize("store", STORES + ["f32"])
def test_pa_gate(store):
    """pa_gate_kernel, y = t * sigmoid(W . t + b) + s with t = the sweep.  A zero W makes the gate a constant and the route EXACT, nothing
    exempt (the matrix product is of zeros): b = +60 -- the gate is 1.0 in fp32, y = t, every value through the load, the product and the
    store unchanged; b = 0 -- exactly 1/2, y = rnd(t / 2) (a tie for every odd subnormal); b = +60 with s = the permuted sweep -- y =
    rnd(t + s), one fp32 add and one rounding.  An identity W makes it t * sigmoid(t): the sweep through the kernel's own sigmoid, held to
    the gates' tolerance against fp64 (a subnormal t read as zero by the matrix core gives the same gate, 1/2).  f32: the bf16 patterns
    widened, against 4 x 2^-24 of the result."""
    from ntire2022_esr_amd import ops
    f32 = store == "f32"
    dt = torch.float32 if f32 else S.DTYPES[store]
    sw, pm = (_sweep("bf16").float(), _perm("bf16").float()) if f32 else (_sweep(store), _perm(store))
    if not f32:
        S.assert_exempt_share(_sweep(store))
    t, s = S.tile(sw, NHW + (C,)), S.tile(pm, NHW + (C,))
    td, sd = t.to(DEV), s.to(DEV)
    pat = rf"pa_gate_kernel<{ {'f32': 0, 'bf16': 1, 'f16': 2}[store] }>"

    def exact(got, want, label):
        if f32:
            bad = ~(got.double() == want.double())
            assert not bool(bad.any()), (label, int(bad.sum()), float(t[bad][0]))
        else:
            S.exact(got, want, dt, v=t.float(), what=label)

    y, name = _traced(pat, lambda: ops.pa_gate(td, *_zero_gate(60.0)))
    exact(y.cpu(), t, f"pa_gate {store} gate 1")
    _report(f"pa_gate {store} W = 0, b = +60: y = t", name, 0)
    y, name = _traced(pat, lambda: ops.pa_gate(td, *_zero_gate(0.0)))
    exact(y.cpu(), (t.float() * 0.5).to(dt), f"pa_gate {store} gate 1/2")
    _report(f"pa_gate {store} W = 0, b = 0: y = t / 2", name, 0)
    y, name = _traced(pat, lambda: ops.pa_gate(td, *_zero_gate(60.0), s=sd))
    pre = t.float() + s.float()
    skip = ~torch.isfinite(pre) | ~torch.isfinite(pre.to(dt).float())       # (a sum beyond the type's range: the ABI requires finite values)
    want = pre.to(dt)
    exact(torch.where(skip, want, y.cpu()), want, f"pa_gate {store} t + s")
    _report(f"pa_gate {store} W = 0, b = +60, s = the permuted sweep: y = rnd(t + s)", name, 0)
    y, name = _traced(pat, lambda: ops.pa_gate(td, torch.eye(C), torch.zeros(C)))
    ref = S.sigmoid_f64(t) * t.double()
    tol = (S.f32_tol(ref) if f32 else S.store_tol(ref, dt)) + S.F32_MIN_NORMAL * t.double().abs()
    worst, share = S.within(y.cpu(), ref, tol, v=t.float(), what=f"pa_gate {store} t sigmoid(t)")
    print(f"pa_gate {store} identity W: {name}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")


@pytest.mark.parametrize("store", STORES)
def test_pa_tail(store):
    """pa_tail_kernel with a centre-tap identity 3x3: t = x = the sweep, through the 3x3's matrix product (x is an MFMA operand there: an x
    that is subnormal in the storage type may be read as zero -- the reference with those inputs zeroed is accepted at those positions and
    nowhere else).  Zero gate weights: b = +60 -- y = rnd(t) = x; b = 0 -- y = rnd(t / 2); b = +60 with s = the permuted sweep -- rnd(t + s):
    all exact.  An identity gate: y = t * sigmoid(rnd(t)), the gates' tolerance against fp64."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n_exempt = S.assert_exempt_share(_sweep(store))
    x, s = S.tile(_sweep(store), NHW + (C,)), S.tile(_perm(store), NHW + (C,))
    xd, sd = x.to(DEV), s.to(DEV)
    w3, b3 = S.identity_weight(C, C, 3), torch.zeros(C)
    pat = rf"pa_tail_kernel<{_bf(store)}, 3>"
    xf = _flush(x)
    n_sub = int(S.is_subnormal(x).sum())
    assert n_sub >= n_exempt
    y, name = _traced(pat, lambda: ops.pa_tail(xd, w3, b3, *_zero_gate(60.0)))
    took = S.exact(y.cpu(), x, dt, v=x.float(), flushed=xf, what=f"pa_tail {store} gate 1")
    _report(f"pa_tail {store} identity 3x3, W = 0, b = +60: y = x", name, took, n_sub)
    y, name = _traced(pat, lambda: ops.pa_tail(xd, w3, b3, *_zero_gate(0.0)))
    took = S.exact(y.cpu(), (x.float() * 0.5).to(dt), dt, v=x.float(), flushed=(xf.float() * 0.5).to(dt), what=f"pa_tail {store} gate 1/2")
    _report(f"pa_tail {store} identity 3x3, W = 0, b = 0: y = x / 2", name, took, n_sub)
    y, name = _traced(pat, lambda: ops.pa_tail(xd, w3, b3, *_zero_gate(60.0), s=sd))
    pre, pre_f = x.float() + s.float(), xf.float() + s.float()
    skip = ~torch.isfinite(pre) | ~torch.isfinite(pre.to(dt).float())
    want = pre.to(dt)
    took = S.exact(torch.where(skip, want, y.cpu()), want, dt, v=x.float(), flushed=pre_f.to(dt), what=f"pa_tail {store} t + s")
    _report(f"pa_tail {store} identity 3x3, W = 0, b = +60, s = the permuted sweep: y = rnd(x + s)", name, took, n_sub)
    y, name = _traced(pat, lambda: ops.pa_tail(xd, w3, b3, torch.eye(C), torch.zeros(C)))
    ref = S.sigmoid_f64(x) * x.double()
    tol = S.store_tol(ref, dt) + S.F32_MIN_NORMAL * x.double().abs()
    got = y.cpu().double()
    flushed = S.flush_mask(x) & (got == 0) & ~((got - ref).abs() <= tol)          # a subnormal x read as zero: t = 0, y = 0
    worst, share = S.within(torch.where(flushed, ref, got), ref, tol, v=x.float(), what=f"pa_tail {store} t sigmoid(t)")
    print(f"pa_tail {store} identity 3x3 and gate: {name}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound); subnormal inputs flushed {int(flushed.sum())} of {n_sub}")


def _listed(fn):
    """a case of this file as the registry module names it: callable(store) runs the case.  A class, because pytest collects a module's
    test_* FUNCTIONS (the cases would run a second time from that module) and warns about any other callable of that name but a class"""
    return type(fn.__name__, (), {"__new__": lambda cls, *args, **kw: fn(*args, **kw), "__doc__": fn.__doc__})


V.SWEPT.update({"pa_gate_kernel": ["test_pa_gate"], "pa_tail_kernel": ["test_pa_tail"]})
V.test_pa_gate, V.test_pa_tail = _listed(test_pa_gate), _listed(test_pa_tail)
