"""-m gpu: every finite 16-bit value through asym_step_kernel (ARFDN's one-launch step) -- through its activation and its stores -- with the
helpers and comparators of tests/test_gpu_value_sweep.py (DESIGN.md "Value sweep").

It lives in a file of its own and ENTERS ITSELF into that module's registry when this file is imported, as tests/test_gpu_sweep_dwrfdn.py
and tests/test_gpu_sweep_repafdn.py do: `SWEPT` gets the kernel, and the test function becomes an attribute of that module, which is where
tests/test_sweep_helper.py::test_every_kernel_is_swept_or_exempt looks for it."""
import pytest
import torch

import _sweep as S
import test_gpu_value_sweep as V
from test_gpu_value_sweep import DEV, LRELU, STORES, _bf, _report, _stage, _sweep, _traced

pytestmark = pytest.mark.gpu
C = 32


def _tap3(vertical):
    """the centre-tap identity of a (3, 1) / (1, 3) convolution over C channels"""
    w = torch.zeros(C, C, 3, 1) if vertical else torch.zeros(C, C, 1, 3)
    o = torch.arange(C)
    w[o, o, 1 if vertical else 0, 0 if vertical else 1] = 1.0
    return w


@pytest.mark.parametrize("store", STORES)
def test_asym_step(store):
    """asym_step_kernel with 0 / 1 weights and ONE non-zero term in the sum, so every stage is exact: a 16-bit value scaled by 0.05 once per
    LeakyReLU it passes, rounded where the kernel rounds.  Terms: `l` -- x -> a_l -> y through the first pair (two matrix products: x and a_l
    are MFMA operands, a subnormal one may be read as zero), `m` -- the second pair, `d` -- x -> d (stored) -> y (d enters the sum as stored,
    not through a matrix product), `in` -- the residual alone, `p` -- an earlier distilled map alone, the input all zeros."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n_exempt = S.assert_exempt_share(_sweep(store))
    n, h, w = S.shape_for(_sweep(store), C)
    x = S.tile(_sweep(store), (n, h, w, C))
    xd, zd = x.to(DEV), torch.zeros_like(x).to(DEV)
    zb = torch.zeros(C)
    z1, zv, zh = torch.zeros(C, C, 1, 1), torch.zeros(C, C, 3, 1), torch.zeros(C, C, 1, 3)
    iv, ih = _tap3(True), _tap3(False)
    n_sub = int(S.is_subnormal(x).sum())
    assert n_sub >= n_exempt
    # term -> (w_d, w_l1, w_l2, w_m1, w_m2, res, input, p1)
    terms = {"l": (z1, iv, ih, zh, zv, False, xd, None), "m": (z1, zv, zh, ih, iv, False, xd, None),
             "d": (S.identity_weight(C, C, 1), zv, zh, zh, zv, False, xd, None), "in": (z1, zv, zh, zh, zv, True, xd, None),
             "p": (z1, zv, zh, zh, zv, False, zd, xd)}
    for term, (wd, wl1, wl2, wm1, wm2, res, inp, p1) in terms.items():
        (dd, y), name = _traced(rf"asym_step_kernel<{_bf(store)}, 1, {'true' if res else 'false'}>",
                                lambda: ops.asym_step(inp, wd, zb, wl1, zb, wl2, zb, wm1, zb, wm2, zb, res=res, p1=p1, act=LRELU, slope=V.SLOPE))
        refs = []
        for flush in (False, True):
            if term in ("l", "m"):
                a16, _ = _stage(x, LRELU, flush)
                d16, y16 = torch.zeros_like(x), _stage(a16, LRELU, flush)[0]
            elif term == "d":
                d16, _ = _stage(x, LRELU, flush)
                y16 = _stage(d16, LRELU, False)[0]
            else:
                d16, y16 = torch.zeros_like(x), _stage(x, LRELU, False)[0]
            refs.append((d16, y16))
        (wd16, wy16), (fd16, fy16) = refs
        label = f"asym step {store} term {term} {n}x{h}x{w}"
        took = S.exact(dd.cpu()[..., :C], wd16, dt, v=x.float(), flushed=fd16, what=label + " d")
        took += S.exact(y.cpu()[..., :C], wy16, dt, v=x.float(), flushed=fy16, what=label + " y")
        _report(label, name, took, 2 * n_sub)


def _listed(fn):
    """a case of this file as the registry module names it: callable(store) runs the case.  A class, because pytest collects a module's
    test_* FUNCTIONS (the cases would run a second time from that module) and warns about any other callable of that name but a class"""
    return type(fn.__name__, (), {"__new__": lambda cls, *args, **kw: fn(*args, **kw), "__doc__": fn.__doc__})


V.SWEPT.update({"asym_step_kernel": ["test_asym_step"]})
V.test_asym_step = _listed(test_asym_step)
