"""CPU-only: the one table that names every launcher (L.LAUNCHERS) against the C dispatch and the library, and the one fill per one-launch op
(ntire2022_esr_amd/descs.py) against the descriptors the tests build by hand.

The engine's op classes and the ops.* wrappers both fill their descriptors through descs.py, so a kernel's own tests and the networks run it
under one field convention.  The independent statement of that convention is the other test files' builders (test_bmdn._step_desc,
_arfdn.step_desc, ...: the baselines of tests/test_fused_limits.py); here each fill, given the operands such a builder wrote, must produce
its descriptor byte for byte."""
import ctypes
import os
import re

import pytest

import test_fused_limits as limits
import test_view_validation as views
from ntire2022_esr_amd import _lib as L, descs

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _read(*path):
    return open(os.path.join(REPO, *path)).read()


def test_table_matches_the_c_dispatch():
    """every `case ESR_OP_X: return fn(&op.FIELD, ...)` of esr_run_ops is the row of that enum value, entry point and field; no other row"""
    enum = {name: int(v) for name, v in re.findall(r"\b(ESR_OP_\w+)\s*=\s*(\d+)", _read("include", "esr_hip.h"))}
    cases = re.findall(r"case\s+(ESR_OP_\w+)\s*:\s*return\s+(\w+)\s*\(\s*&op\.(\w+)\s*,", _read("ntire2022_esr_amd", "csrc", "esr_hip.hip"))
    assert len(cases) == len(enum) == 24 and {c[0] for c in cases} == set(enum)
    assert {enum[name]: (fn, field) for name, fn, field in cases} == {kind: row[:2] for kind, row in L.LAUNCHERS.items()}
    for name, kind in enum.items():                         # the binding's constants are the header's
        assert getattr(L, name.removeprefix("ESR_")) == kind


def test_table_matches_the_library():
    """every launcher and predicate is a declared export and is typed, by lib(), with a pointer to the descriptor class of its Op field"""
    lib, fields = L.lib(), dict(L.Op._fields_)
    for kind, (fn, field, predicate) in L.LAUNCHERS.items():
        assert fn in L.EXPORTS and (predicate is None or (predicate in L.EXPORTS and predicate.endswith("_supported"))), kind
        assert getattr(lib, fn).argtypes == [ctypes.POINTER(fields[field]), ctypes.c_void_p] and getattr(lib, fn).restype is ctypes.c_int, fn
        if predicate is not None:
            assert getattr(lib, predicate).argtypes == [ctypes.POINTER(fields[field])] and getattr(lib, predicate).restype is ctypes.c_int, predicate


A, S, M, V = limits.A, limits.S, 0x10000000, L.View        # the stand-in addresses of the baselines' builders
BF16, F16 = L.STORE["bf16"], L.STORE["f16"]


def _filled(cls, fill, *args, **kw):
    d = cls()
    fill(d, *args, **kw)
    return d


def _pa_tail():
    d = FILLS["pa_gate"]()
    descs.pa_tail(d, x=V(A, 48, 0), w3=A, w=A)
    return d


def _prelu(store):
    return _filled(L.ConvDesc, descs.prelu, (1, 4, 4), L.STORE[store], srcs=[(V(M, 96, 0), 41)], a=M + 0x900000, y=V(M + 0x800000, 96, 0))


def _mdsa(planar):
    return _filled(L.ConvDesc, descs.mdsa_gate, (1, 4, 4), BF16, f=V(M, 64 if planar else 192, 0), x=V(M + 0x400000, 64, 0), w=M + 0x900000, cin=192,
                   cout=64, y=V(M + 0x800000, 64, 0), seg=(0x1000, 4) if planar else None)


_CHAIN = dict(x=views.V(48, 8), cin=48, cout=48, act=L.ACT_LRELU, slope=0.05)
# name (of limits.ENTRIES) -> the fill, called with the operands that entry's base() builder wrote by hand
FILLS = {
    "pa_gate": lambda: _filled(L.ConvDesc, descs.pa_gate, (1, 32, 40), BF16, t=V(A, 48, 0), w=A, c=48, y=V(A + 2 * S, 48, 0), y_width=48, s=V(A + S, 48, 0)),
    "pa_tail": _pa_tail,
    "conv_prelu": lambda: _filled(L.ConvDesc, descs.conv_prelu, (1, 4, 4), BF16, x=V(M, 64, 0), w=M + 0x900000, a=M + 0xa00000, cin=64, cout=64,
                                  y=V(M + 0x800000, 64, 0)),
    "mdsa_gate": lambda: _mdsa(False),
    "mdsa_gate_planar": lambda: _mdsa(True),
    "asym_step": lambda: _filled(L.ConvDesc, descs.asym_step, (1, 32, 40), BF16, x=V(A, 32, 0), w_d=A, w_taps=A, cin=25, c=25, act=L.ACT_LRELU, slope=0.05,
                                 res=True, dd=V(A + 2 * S, 128, 32), y=V(A + S, 32, 0), y_width=25, p=[V(A + 2 * S, 128, 64), V(A + 2 * S, 128, 96)]),
    "prelu": lambda: _prelu("bf16"),
    "prelu_f32": lambda: _prelu("f32"),
    "resdb_step": lambda: _filled(L.ConvDesc, descs.resdb_step, (1, 4, 4), BF16, x=V(A, 48, 0), a=A, w_e=A, w_c=A, cin=48, cout=48, extra_channels=0,
                                  dists=V(A + 2 * S, 16, 0), dists_channels=16, y=V(A + S, 48, 0)),
    "cx_block": lambda: _filled(L.ChainDesc, descs.cx_block, (1, 32, 40), BF16, v=V(A, 56, 0), w0=A, w1=A, w2=A, c=50, m=200, cout=50, slope=0.05,
                                out=V(A + 4096, 56, 0), out_width=56),
    "dwpw_pair": lambda: _filled(L.ChainDesc, descs.dwpw_pair, (1, 32, 40), BF16, x=V(A, 56, 0), w=[A] * 4, c=50, slope=0.05, out=V(A + 4096, 56, 0),
                                 out_width=56),
    "refine_cascade": lambda: _filled(L.ChainDesc, descs.refine_cascade, (1, 32, 40), BF16, d2=V(A, 32, 0), w=[A] * 4, cin=32, cmid=16, cout=16, slope=0.05,
                                      d3=V(A + 4096, 32, 0), d3_width=16, r4=V(A + 4096, 32, 16), r4_width=16),
    "distill_step": lambda: _filled(L.ChainDesc, descs.distill_step, (1, 32, 40), BF16, x=V(A, 40, 0), w_d=A, w_fold=A, cin=40, cmid=20, cout=20, res=False,
                                    dd=V(A, 32, 0), d_width=20, y=V(A, 32, 0), y_width=32),
    "resblock_head": lambda: _filled(L.ConvDesc, descs.resblock_head, (1, 32, 40), F16, x=V(A, 32, 0), g=V(A + 64, 32, 0), xs=V(A + 128, 32, 0), w1=A, w2=A,
                                     wc=A, cin=32, cout=32, u=V(A + 192, 32, 0), c1=V(A, 16, 0), c1_width=16),
    "hfab": lambda: _filled(L.ChainDesc, descs.hfab, (1, 16, 16), BF16, **_CHAIN, w=[views.A] * 4, cmid=16, y=views.V(48, 8, 1), y_width=48),
    "chain": lambda: _filled(L.ChainDesc, descs.chain, (1, 16, 16), BF16, **_CHAIN, w=[views.A] * 3, cmid=48, res_mode=L.RES_POST_ACT, post_w=views.A,
                             v=views.V(48, 8, 1), v_width=48, post_act=L.ACT_NONE, post2_w=views.A, c1=views.V(16, 8, 2), c1_width=16),
}


def test_every_baseline_has_its_fill():
    assert set(FILLS) == set(limits.ENTRIES) and len(FILLS) == 16


@pytest.mark.parametrize("name", sorted(FILLS))
def test_fill_matches_the_hand_built_descriptor(name):
    want, got = limits.ENTRIES[name]["base"](), FILLS[name]()
    assert type(got) is type(want)
    assert bytes(got) == bytes(want), [f for f, _ in type(want)._fields_ if _raw(got, f) != _raw(want, f)]


def _raw(d, name):
    """the bytes of one field of a descriptor"""
    at = getattr(type(d), name)
    return bytes(d)[at.offset:at.offset + at.size]
